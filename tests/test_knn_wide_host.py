"""CPU tests of pcc_knn's size contract for the wide path (k up to 128, any channel count): sizes are validated before
anything touches the device, so these run without a GPU."""

PCC_EINVAL = -22


def _knn_status(b, c, n, k):
    from pointcloudcounterfactual_amd import _lib

    rc = _lib.lib.pcc_knn(b, c, n, k, None, None, None)
    return rc, _lib.lib.pcc_last_error().decode()


def test_wide_k_and_many_channels_pass_the_size_checks():
    """k in (32, 128] and c > 128 are accepted sizes: with null pointers the call fails on the pointers, not the sizes."""
    for b, c, n, k in ((1, 3, 300, 40), (1, 256, 300, 20), (2, 1024, 200, 128), (1, 64, 128, 128), (1, 4096, 10, 1)):
        rc, msg = _knn_status(b, c, n, k)
        assert rc == PCC_EINVAL, (b, c, n, k)
        assert 'null pointer' in msg, (b, c, n, k, msg)


def test_k_above_128_is_refused():
    rc, msg = _knn_status(1, 3, 300, 129)
    assert rc == PCC_EINVAL
    assert '128' in msg and 'null pointer' not in msg, msg
    rc, msg = _knn_status(1, 300, 1000, 500)
    assert rc == PCC_EINVAL and '128' in msg, msg


def test_k_above_n_is_still_refused_first():
    rc, msg = _knn_status(1, 3, 40, 41)
    assert rc == PCC_EINVAL and 'exceeds' in msg, msg


def _knn_cross_status(b, c, nq, n, k):
    from pointcloudcounterfactual_amd import _lib

    rc = _lib.lib.pcc_knn_cross(b, c, nq, n, k, None, None, None, None, None)
    return rc, _lib.lib.pcc_last_error().decode()


def test_every_entry_check_of_pcc_knn_keeps_its_status_and_text():
    """Null pointers throughout: every check runs before anything touches the device, in this order."""
    bad = (PCC_EINVAL, 'knn: bad size')
    for sizes, expect in (
            ((-1, 3, 10, 1), bad), ((1, 0, 10, 1), bad), ((1, 3, -1, 1), bad), ((1, 3, 10, 0), bad),
            ((0, 3, 10, 11), (0, '')), ((1, 3, 0, 5), (0, '')), ((0, 3, 0, 500), (0, '')),
            ((1, 3, 40, 41), (PCC_EINVAL, 'knn: k exceeds the number of points (torch.topk raises too)')),
            ((70000, 3, 100, 200), (PCC_EINVAL, 'knn: k exceeds the number of points (torch.topk raises too)')),
            ((1, 3, 300, 129), (PCC_EINVAL, 'knn: k > 128 is not supported')),
            ((65536, 3, 300, 129), (PCC_EINVAL, 'knn: k > 128 is not supported')),
            ((65536, 3, 300, 5), (PCC_EINVAL, 'knn: batch too large')),
            ((65535, 3, 300, 5), (PCC_EINVAL, 'knn: null pointer')),
            ((1, 64, 128, 128), (PCC_EINVAL, 'knn: null pointer'))):
        assert _knn_status(*sizes) == expect, sizes


def test_every_entry_check_of_pcc_knn_cross_keeps_its_status_and_text():
    bad = (PCC_EINVAL, 'knn_cross: bad size')
    many = 65535 * 128 + 1
    for sizes, expect in (
            ((-1, 3, 10, 10, 1), bad), ((1, 0, 10, 10, 1), bad), ((1, 3, -1, 10, 1), bad), ((1, 3, 10, -1, 1), bad),
            ((1, 3, 10, 10, 0), bad),
            ((0, 3, 10, 10, 11), (0, '')), ((1, 3, 0, 5, 6), (0, '')), ((1, 3, 0, 0, 1), (0, '')),
            ((1, 3, 50, 40, 41), (PCC_EINVAL, 'knn_cross: k exceeds the number of candidates (torch.topk raises too)')),
            ((1, 3, 5, 0, 1), (PCC_EINVAL, 'knn_cross: k exceeds the number of candidates (torch.topk raises too)')),
            ((1, 3, 10, 300, 129), (PCC_EINVAL, 'knn_cross: k > 128 is not supported')),
            ((65536, 3, 40000, 300, 129), (PCC_EINVAL, 'knn_cross: k > 128 is not supported')),
            ((65536, 3, 40000, 300, 5), (PCC_EINVAL, 'knn_cross: batch too large')),
            ((65535, 4, 32769, many, 5), (PCC_EINVAL, 'knn_cross: too many queries (b * nq >= 2^31)')),
            ((32768, 3, 65536, 300, 5), (PCC_EINVAL, 'knn_cross: too many queries (b * nq >= 2^31)')),
            ((1, 4, 10, many, 5), (PCC_EINVAL, 'knn_cross: too many candidates for c >= 4 (n > 65535 * 128)')),
            ((1, 3, 10, many, 5), (PCC_EINVAL, 'knn_cross: null pointer')),
            ((1, 4, 10, many - 1, 5), (PCC_EINVAL, 'knn_cross: null pointer')),
            ((65535, 64, 32768, 128, 128), (PCC_EINVAL, 'knn_cross: null pointer'))):
        assert _knn_cross_status(*sizes) == expect, sizes


def test_knn_wide_switch_is_known():
    from pointcloudcounterfactual_amd import _lib

    assert _lib.TUNING['knn_wide'] == 9
