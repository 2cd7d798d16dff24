"""Which kernel a ``pcc_knn`` call runs, restated from the dispatch rules in DESIGN.md and the kernel headers
(csrc/knn.hip, knn.hpp, knn_mfma.hip) -- never obtained from the library.  The names are the exact launch-profile names:
they carry the template instantiation."""

SLOTS = (4, 8, 16, 20, 25, 32)    # list widths K of the instantiations: a call takes the fewest slots >= k
CPS = (8, 16, 32, 64, 128)        # padded channel counts of the MFMA kernels (the role-split kernel starts at 16)
SORTED_MAX_N = 16384              # c <= 3: the sorted search up to here, the exhaustive kernel behind it
SPLIT_QUERIES = 256               # queries per workgroup of the role-split kernel
FAMILIES = ('knn_sorted_kernel', 'knn_small_kernel', 'knn_mfma_kernel', 'knn_mfma_split_kernel', 'knn_wide_')


def slots(k):
    return next(s for s in SLOTS if s >= k)


def padded(c, least=8):
    return next(p for p in CPS if p >= max(c, least))


def kernel_of(b, c, n, k, cus=256, nosplit=0, wide=0):
    """The search kernel of ``pcc_knn(b, c, n, k)`` on a device of ``cus`` compute units under the switches knn_nosplit
    (1 = the 128-query MFMA kernel everywhere, 2 = the role-split kernel everywhere) and knn_wide (1 = the wide path
    everywhere).  The wide path is named by its selection kernel (its distance kernel runs too where c > 3)."""
    if k > 32 or c > 128 or wide == 1:
        return wide_select(c, k)
    if c <= 3:
        return f'knn_sorted_kernel<{slots(k)}>' if n <= SORTED_MAX_N else f'knn_small_kernel<{slots(k)},4>'
    # the role-split kernel once its 256-query workgroups fill three quarters of the chip (and its selection log, 512 KB
    # per workgroup, stays under 1 GiB)
    groups = -(-n // SPLIT_QUERIES) * b
    split = nosplit == 2 or (nosplit == 0 and groups * 4 >= 3 * cus and groups * (512 << 10) <= 1 << 30)
    if split:
        return f'knn_mfma_split_kernel<{slots(k)},{padded(c, 16)}>'
    return f'knn_mfma_kernel<{slots(k)},{padded(c)},1>'


def wide_select(c, k, sliced=False):
    """The selection kernel of the wide path and of ``pcc_knn_cross``: <list slots, source of the keys> -- 64 slots up to
    k = 64, 128 above; exact difference-form distances computed on the fly where c <= 3 ('diff'), rows of the distance
    kernel's matrix otherwise ('rows').  ``sliced``: the candidate axis is cut into slices, whose partial lists a second
    launch (``wide_merge``) merges; the self search never slices."""
    return f"knn_wide_select_kernel<{64 if k <= 64 else 128},{'diff' if c <= 3 else 'rows'}>" + (' sliced' if sliced else '')


def wide_merge(k):
    return f'knn_wide_select_kernel<{64 if k <= 64 else 128},keys>'


def cross_slices(rows, n, cus, forced=0):
    """Slices of the candidate axis of one ``pcc_knn_cross`` launch of ``rows`` queries over ``n`` candidates: one wave per
    query fills the chip from 8 waves per CU on; below that enough slices to get there, at most 64 and none shorter than
    2048 candidates; knn_cross_split = S >= 1 forces S.  Whole blocks of 256 candidates per slice, no empty slice."""
    want = forced if forced >= 1 else 1 if rows >= 8 * cus else max(1, min(-(-8 * cus // rows), 64, n // 2048))
    length = -(-(-(-n // want)) // 256) * 256
    return -(-n // length)
